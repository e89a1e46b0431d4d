"""GPU: ops.track_infill (poco_op_track_infill, csrc/track_infill.hip) against its float64 numpy restatement tests/infill_np.py on
seeded random proper rotations.

Tracks of 1, 2, 3, 63, 64, 65, 127, 128, 129 and 200 rows in one ragged call and each alone: the sizes at which a chunk carry (the
kernel walks a track in chunks of 64 rows), a wave edge or a track boundary can go wrong.  Every column of a track carries one
reliability pattern (COLUMNS below).  Flags and touched rows are exact; entries with flag 0, 2, 3 are bit-exact (against the input
or the anchor row); flag-1 entries lie within one fp32 ulp at 1.0 (2^-23) of the restatement rounded to fp32: both sides evaluate
the same float64 formula, and differing acos / sin implementations move a value by ~1e-15, which can only flip the final rounding.
The outputs lie between poisoned guard bands."""
import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import infill_np as inp

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)
THR = np.float32(0.5)
GAP = 16                      # the small max_gap; the exact-gap columns are built for it
DENSE = 40                    # rows of a track whose frame indices are consecutive; holes of up to two frames follow
L = 14
ULP1 = 2.0 ** -23
GUARD = 256                   # bytes on either side of every output
POISON = 0xA5

COLUMNS = {0: "random runs (moves the linear block)", 1: "all reliable", 2: "none reliable", 3: "a run at the head", 4: "a run at the tail",
           5: "rows 40 .. 150: from chunk 0 into chunk 2", 6: "alternating", 7: "anchors exactly GAP frames apart",
           8: "anchors GAP + 1 frames apart", 9: "NaN uncertainties", 10: "runs at head and tail: the neighbour's rows are nearer",
           23: "one constant rotation: near-identical anchors"}


def _runs(r, T, frac=0.1):
    """About `frac` of the rows unreliable, in runs of 1 .. 12 rows."""
    bad = np.zeros(T, bool)
    while bad.mean() < frac:
        t = int(r.integers(0, T))
        bad[t:t + int(r.integers(1, 13))] = True
    return bad


def _track(r, T):
    pose = inp.smooth_rotations(r, T, 1.0)               # <= 1 degree a row: anchors 169 rows apart stay below 170 degrees
    pose[:, 11:23] = inp.smooth_rotations(r, T, 8.0)[:, 11:23]   # the columns of short random runs turn faster (checked below)
    pose[:, 23] = pose[0, 23]
    frames = int(r.integers(0, 1000)) + np.cumsum(np.where(np.arange(T) < DENSE, 1, r.integers(1, 4, T)))
    bad = np.stack([_runs(r, T) for _ in range(24)], 1)
    rows = np.arange(T)
    bad[:, 1] = False
    bad[:, 2] = True
    bad[:, 3] = rows < 5
    bad[:, 4] = rows >= T - 5
    bad[:, 5] = (rows >= 40) & (rows <= 150)
    bad[:, 6] = rows % 2 == 1
    bad[:, 7] = (rows >= 3) & (rows <= GAP + 1)          # anchors at rows 2 and GAP + 2 (consecutive frames there)
    bad[:, 8] = (rows >= 3) & (rows <= GAP + 2)          # ... and GAP + 3
    bad[:, 10] = (rows < 3) | (rows >= T - 3)
    u = np.where(bad, r.uniform(0.5001, 2.0, (T, 24)), r.uniform(0.0, 0.5, (T, 24))).astype(np.float32)
    u[(~bad) & (r.random((T, 24)) < 0.1)] = THR           # u == thresh is reliable
    nan = _runs(r, T, 0.15)
    u[nan, 9] = np.nan
    lin = r.standard_normal((T, L)).astype(np.float32)
    return pose, u, frames.astype(np.int32), lin


@pytest.fixture(scope="module")
def data():
    r = np.random.default_rng(11)
    parts = [_track(r, T) for T in LENGTHS]
    pose, u, frames, lin = (np.concatenate([p[i] for p in parts]) for i in range(4))
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    return dict(pose=pose, u=u, frames=frames, offsets=offsets, lin=lin)


_REF = {}


def _ref(data, max_gap):
    if max_gap not in _REF:
        _REF[max_gap] = inp.infill(**data, thresh=THR, max_gap=max_gap)
    return _REF[max_gap]


def _guarded(shape, dtype, dev):
    """A contiguous tensor of `shape` inside one allocation, GUARD poisoned bytes before and after it, itself poisoned too (an
    element the kernel leaves out shows)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pad = -n % 16
    flat = torch.full((GUARD + n + pad + GUARD,), POISON, dtype=torch.uint8, device=dev)
    return flat, flat[GUARD:GUARD + n].view(dtype).view(shape)


def _bands_intact(flat, body):
    n = body.numel() * body.element_size()
    return bool((flat[:GUARD] == POISON).all()) and bool((flat[GUARD + n:] == POISON).all())


def _run(d, max_gap, dev, guarded=True):
    N = d["pose"].shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                               # noqa: E731
    out = bufs = None
    if guarded:
        bufs = [_guarded(s, dt, dev) for s, dt in (((N, 24, 3, 3), torch.float32), ((N, L), torch.float32), ((N, 24), torch.uint8),
                                                   ((N,), torch.uint8), ((N,), torch.int32), ((1,), torch.int32))]
        out = [b for _, b in bufs]
    res = ops.track_infill(t(d["pose"]), t(d["u"]), t(d["frames"]), torch.from_numpy(d["offsets"]), t(d["lin"]), float(THR), max_gap,
                           rows=True, out=out)
    torch.cuda.synchronize()
    if guarded:
        for flat, body in bufs:
            assert _bands_intact(flat, body)
    names = ("pose", "lin", "flags", "touched", "rows", "count")
    return {k: v.cpu().numpy() for k, v in zip(names, res)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(got, ref, d, max_gap):
    """The conditions of the module docstring; returns the largest deviation of a flag-1 matrix entry and of a lin entry in ulps."""
    assert np.array_equal(got["flags"], ref["flags"]) and np.array_equal(got["touched"], ref["touched"])
    n = int(got["count"][0])
    assert n == int(ref["touched"].sum()) and np.array_equal(got["rows"][:n], np.nonzero(ref["touched"])[0])
    assert (got["rows"][n:].view(np.uint8) == POISON).all()                     # the rest of the list is left alone
    f = ref["flags"]
    for flag in (0, 3):                                                         # against the input
        assert np.array_equal(_bits(got["pose"])[f == flag], _bits(d["pose"])[f == flag]), flag
    assert np.array_equal(_bits(got["pose"])[f == 2], _bits(ref["pose"])[f == 2])        # the restatement copies the anchor row
    for t, j in zip(*np.nonzero(f == 2)):                                       # ... which is a row of the input, in the same track
        p = int(np.searchsorted(d["offsets"], t, side="right")) - 1
        lo, hi = d["offsets"][p], d["offsets"][p + 1]
        same = (_bits(d["pose"])[lo:hi, j].reshape(hi - lo, 9) == _bits(got["pose"])[t, j].reshape(9)).all(1)
        assert same.any()
    dev1 = np.abs(got["pose"].astype(np.float64) - ref["pose"].astype(np.float64))[f == 1]
    worst = float(dev1.max()) if dev1.size else 0.0
    assert worst <= ULP1, worst
    # the linear block follows column 0
    f0 = f[:, 0]
    keep = (f0 == 0) | (f0 == 3)
    assert np.array_equal(_bits(got["lin"])[keep], _bits(d["lin"])[keep]) and np.array_equal(_bits(got["lin"])[f0 == 2], _bits(ref["lin"])[f0 == 2])
    dl = np.abs(got["lin"].astype(np.float64) - ref["lin"].astype(np.float64))[f0 == 1]
    ulp = np.spacing(np.abs(ref["lin"][f0 == 1]))
    worst_lin = float((dl / ulp).max()) if dl.size else 0.0
    assert worst_lin <= 1.0, worst_lin
    return worst / ULP1, worst_lin


@pytest.mark.parametrize("max_gap", [GAP, 1000])
def test_ragged_call_matches_the_restatement(data, max_gap, cuda):
    ref = _ref(data, max_gap)
    f = ref["flags"]
    # the material is what the docstring says: every flag occurs, the patterns land as planned
    assert {int(x) for x in np.unique(f)} == {0, 1, 2, 3}
    assert not f[:, 1].any() and (f[:, 2] == 3).all()
    big = int(data["offsets"][-2])                                               # the 200-row track
    run = {int(x) for x in np.unique(f[big + 40:big + 151, 5])}                  # the run over two chunk edges: interpolated when the
    assert run == ({1} if max_gap == 1000 else {2, 3})                           # gap allows, else held near its ends and left between
    if max_gap == GAP:
        for lo in data["offsets"][3:-1]:                                         # tracks of 63 rows and more
            assert (f[lo + 3:lo + GAP + 2, 7] == 1).all() and not (f[lo + 3:lo + GAP + 3, 8] == 1).any()
    for j in range(24):                                                          # the shortest arc is well defined
        for t in np.nonzero(f[:, j] == 1)[0]:
            p = int(np.searchsorted(data["offsets"], t, side="right")) - 1
            _, a, b, _, _ = inp.decide(data["frames"], data["u"][:, j] <= THR, t, int(data["offsets"][p]), int(data["offsets"][p + 1]), max_gap)
            assert inp.relative_angle_deg(data["pose"][a, j], data["pose"][b, j]) <= 170.0
    got = _run(data, max_gap, cuda)
    worst, worst_lin = _check(got, ref, data, max_gap)
    print(f"track_infill max_gap={max_gap}: {int((f == 1).sum())} interpolated entries, largest deviation {worst:.3f} ulp(1.0) "
          f"on the matrices, {worst_lin:.3f} ulp on the linear block")
    # the same call again: the same bits
    again = _run(data, max_gap, cuda)
    for k in ("pose", "lin", "flags", "touched"):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("max_gap", [GAP, 1000])
def test_each_track_alone_gives_the_same_bits(data, max_gap, cuda):
    """One call per track (another grid, other row numbers) = the rows of the ragged call, bit for bit, and the restatement on the
    track alone."""
    whole = _run(data, max_gap, cuda, guarded=False)
    ref = _ref(data, max_gap)
    off = data["offsets"]
    for p, T in enumerate(LENGTHS):
        lo, hi = int(off[p]), int(off[p + 1])
        d = dict(pose=data["pose"][lo:hi], u=data["u"][lo:hi], frames=data["frames"][lo:hi], offsets=np.array([0, T], np.int32),
                 lin=data["lin"][lo:hi])
        got = _run(d, max_gap, cuda)
        for k in ("pose", "lin", "flags", "touched"):
            assert np.array_equal(got[k].view(np.uint8), whole[k][lo:hi].view(np.uint8)), (T, k)
        sub = {k: ref[k][lo:hi] for k in ("pose", "lin", "flags", "touched")}
        _check(got, sub, d, max_gap)


def test_all_reliable_and_none_reliable_are_the_input(data, cuda):
    for value, flag in ((0.0, 0), (1.0, 3), (np.nan, 3)):
        d = dict(data, u=np.full_like(data["u"], value))
        got = _run(d, GAP, cuda)
        assert np.array_equal(_bits(got["pose"]), _bits(d["pose"])) and np.array_equal(_bits(got["lin"]), _bits(d["lin"]))
        assert (got["flags"] == flag).all() and not got["touched"].any() and int(got["count"][0]) == 0


def test_argument_errors(data, cuda):
    from poco_amd._lib import PocoHipError
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)                              # noqa: E731
    N = data["pose"].shape[0]
    base = dict(pose=t(data["pose"]), u=t(data["u"]), frames=t(data["frames"]), offsets=torch.from_numpy(data["offsets"]), lin=t(data["lin"]),
                thresh=0.5, max_gap=8)
    bad_off = data["offsets"].copy()
    bad_off[3] = bad_off[2]
    for kw in (dict(pose=base["pose"][:, :23]), dict(pose=base["pose"].double()), dict(u=base["u"][:-1]), dict(u=base["u"].half()),
               dict(frames=base["frames"].long()), dict(frames=base["frames"][:-1]), dict(lin=torch.zeros(N, 17, device=cuda)),
               dict(lin=base["lin"][:-1]), dict(max_gap=0), dict(max_gap=2.5), dict(offsets=torch.from_numpy(bad_off)),
               dict(offsets=torch.from_numpy(data["offsets"][:-1].copy())), dict(offsets=torch.from_numpy(data["offsets"]).long()),
               dict(offsets=torch.from_numpy(data["offsets"][1:].copy()))):
        with pytest.raises(PocoHipError, match="track_infill"):
            ops.track_infill(**{**base, **kw})
