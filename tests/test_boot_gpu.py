"""poco_op_bootstrap on the GPU against tests/boot_np.py (include/poco_hip.h): draw_counts element for element;
center, unit_mom and out within terms x 2^-52 x sum |terms| of math.fsum (not bitwise: the device adds in its own fixed order); a NaN
or an infinity exactly where the yardstick has one; every output bitwise independent of max_blocks and equal from run to run; inputs
unchanged; outputs between guard words; poisoned outputs untouched on the error paths.

Each stage is held against the yardstick fed the device's result of the stage before (unit_mom from the device's center, out from the
device's unit_mom), so that every bound is the rounding of that stage's own additions:
  center    n additions and a division:                  (n + 2) x 2^-52 x sum |v| / n
  unit_mom  per term two subtractions and a product (1.5 ulp), then `rows` additions:   (rows + 4) x 2^-52 x sum |terms|
  out       U additions:                                 (U + 1) x 2^-52 x sum |unit_mom[idx]|"""
import functools

import numpy as np
import pytest

from tests import boot_np

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
G = 64                                                                    # guard words on either side of every output
DFILL, IFILL = -7.25, -77
WORST = {"center": 0.0, "unit_mom": 0.0, "out": 0.0}                      # the largest |error| / bound seen, printed per test


def pairs_of(E, P):
    """P pairs over E planes; with P >= 2 the second names one plane twice, with P = 16 every third does."""
    if P == 1:
        return [(0, E - 1)]
    return [((3 * k) % E, (3 * k) % E if k % 3 == 1 else (5 * k + 1) % E) for k in range(P)]


def units_of(kind, n):
    """unit_offsets [U + 1] (None: every row its own unit) of n rows."""
    if kind == "null":
        return None
    if kind == "ones":
        return np.arange(n + 1)
    if kind == "one":
        return np.asarray([0, n])
    if kind == "sel24":                                                   # |sel| = 24 rows per crop (n a multiple of 24)
        assert n % 24 == 0
        return np.arange(n // 24 + 1) * 24
    assert kind == "ragged"                                               # sizes 1..300, empty units first, last and adjacent
    r = np.random.default_rng(n)
    sizes = [0, 0]
    while sum(sizes) < n:
        sizes.append(int(min(r.integers(1, 301), n - sum(sizes))))
        if len(sizes) % 4 == 0:
            sizes += [0, 0]
    return np.concatenate([[0], np.cumsum(sizes + [0])])


def values_of(kind, E, n, seed=0):
    r = np.random.default_rng([seed, E, n])
    x = r.standard_normal((E, n)).astype(np.float32)
    if kind == "equal":
        x[:] = np.float32(0.3)
    elif kind == "offset":
        x = (1e6 + x).astype(np.float32)
    elif kind == "denormal":
        x = (x * np.float32(1e-40)).astype(np.float32)
        assert np.any((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny))
    elif kind == "nan":
        x[0, n // 2] = np.nan
    elif kind == "inf":
        x[E - 1, n // 3] = np.inf
    else:
        assert kind == "normal"
    return x


def run(cuda, planes, pairs, offsets, B, seed, max_blocks=0):
    """One ops.bootstrap call into guarded, poisoned outputs -> host arrays.  Checks the guards and that the inputs are only read."""
    import torch
    from poco_amd import ops
    E, n = planes.shape
    U = n if offsets is None else len(offsets) - 1
    M = 1 + E + len(pairs)
    dp = torch.from_numpy(np.array(planes, np.float32)).to(cuda)
    do = None if offsets is None else torch.from_numpy(np.asarray(offsets, np.int32)).to(cuda)
    keep = [t.clone() for t in (dp, do) if t is not None]
    sizes = {"center": E, "unit_mom": U * M, "out": (B + 1) * M, "draw_counts": B * U}
    raw = {k: torch.full((v + 2 * G,), IFILL if k == "draw_counts" else DFILL, device=cuda, dtype=torch.int32 if k == "draw_counts" else torch.float64)
           for k, v in sizes.items()}
    shapes = {"center": (E,), "unit_mom": (U, M), "out": (B + 1, M), "draw_counts": (B, U)}
    out = {k: raw[k][G:G + sizes[k]].view(shapes[k]) for k in raw}
    ops.bootstrap(dp, pairs, do, B, seed, max_blocks, out=out)
    torch.cuda.synchronize()
    for t, k in zip([t for t in (dp, do) if t is not None], keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    host = {k: v.cpu().numpy() for k, v in raw.items()}
    for k, v in host.items():
        fill = IFILL if k == "draw_counts" else DFILL
        assert np.all(v[:G] == fill) and np.all(v[len(v) - G:] == fill), k
    return {k: host[k][G:G + sizes[k]].reshape(shapes[k]) for k in host}


def same_bits(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


def close(name, got, want, bound):
    """NaN and infinities exactly where the yardstick has them, the finite words within the bound."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape, name
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.any(np.isinf(got[~inf & ~np.isnan(got)])), name
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= bound[fin]), (name, float(np.max(err - bound[fin])))
    WORST[name] = max(WORST[name], float(np.max(err / np.maximum(bound[fin], 1e-300), initial=0.0)))


def check(got, planes, pairs, offsets, B, seed):
    E, n = planes.shape
    U = n if offsets is None else len(offsets) - 1
    cw, cmag = boot_np.centers(planes)
    close("center", got["center"], cw, (n + 2) * EPS * cmag)
    mw, mmag = boot_np.unit_moments(planes, pairs, offsets, got["center"])
    assert np.array_equal(got["unit_mom"][:, 0], mw[:, 0])                                     # the row counts are exact
    close("unit_mom", got["unit_mom"], mw, (mw[:, :1] + 4) * EPS * mmag)
    ow, omag, counts = boot_np.resample(got["unit_mom"], B, seed)
    assert np.array_equal(got["draw_counts"], counts) and np.all(counts.sum(axis=1) == U)
    assert np.array_equal(got["out"][:, 0], ow[:, 0]) and got["out"][0, 0] == n                # sums of small integers are exact
    close("out", got["out"], ow, (U + 1) * EPS * omag)                                         # row 0: the column sums of unit_mom
    print("largest |error| / bound so far:", WORST)


# (n, units, B, (E, P)): every n, every kind of units, every B and every (E, P) of the issue at least once; the yardstick is plain
# Python, so the large n go with few columns and few replicates
SHAPES = [(1, "null", 3, (3, 1)), (2, "null", 3, (3, 1)), (63, "null", 1, (1, 0)), (64, "null", 3, (3, 1)), (65, "null", 257, (3, 1)),
          (255, "null", 3, (3, 1)), (256, "null", 0, (3, 1)), (257, "null", 3, (16, 16)), (4099, "null", 3, (3, 1)),
          (1, "ones", 1, (1, 0)), (1, "one", 3, (16, 16)), (65, "ones", 3, (3, 1)), (64, "one", 257, (1, 0)), (257, "one", 3, (3, 1)),
          (4099, "one", 1, (3, 1)), (63, "ragged", 0, (16, 16)), (255, "ragged", 257, (3, 1)), (257, "ragged", 3, (16, 16)),
          (4099, "ragged", 3, (3, 1)), (24 * 11, "sel24", 3, (16, 16)), (24 * 171, "sel24", 257, (1, 0)), (2, "one", 0, (1, 0)),
          (256, "ragged", 1, (3, 1))]


@functools.lru_cache(maxsize=None)
def case(n, units, E, P, values="normal"):
    planes, offsets = values_of(values, E, n), units_of(units, n)
    planes.setflags(write=False)
    return planes, pairs_of(E, P), offsets


@pytest.mark.parametrize("n,units,B,EP", SHAPES)
def test_shapes(cuda, n, units, B, EP):
    planes, pairs, offsets = case(n, units, *EP)
    got = run(cuda, planes, pairs, offsets, B, 3)
    check(got, planes, pairs, offsets, B, 3)
    for mb in (1, 7, 0):                                                  # the grid does not matter, nor does the run
        same_bits(got, run(cuda, planes, pairs, offsets, B, 3, mb))


def test_explicit_units_of_one_row_are_the_default(cuda):
    planes, pairs, _ = case(257, "null", 3, 1)
    same_bits(run(cuda, planes, pairs, None, 5, 11), run(cuda, planes, pairs, np.arange(258), 5, 11))


def test_a_large_sample(cuda):
    n, B = 70001, 8
    planes, pairs, offsets = case(n, "null", 1, 1)                       # one plane and its square: the yardstick is plain Python
    got = run(cuda, planes, pairs, offsets, B, 2 ** 63 + 5)
    check(got, planes, pairs, offsets, B, 2 ** 63 + 5)
    same_bits(got, run(cuda, planes, pairs, offsets, B, 2 ** 63 + 5, 7))


@pytest.mark.parametrize("values", ["normal", "equal", "offset", "denormal", "nan", "inf"])
@pytest.mark.parametrize("units", ["null", "ragged"])
def test_values(cuda, values, units):
    n, B, seed = 257, 9, 1
    planes, offsets = values_of(values, 3, n, seed=7), units_of(units, n)
    pairs = [(0, 2), (1, 1), (0, 0), (2, 2)]
    got = run(cuda, planes, pairs, offsets, B, seed)
    check(got, planes, pairs, offsets, B, seed)
    if values in ("nan", "inf"):
        # plane and row of the bad value: its raw column is bad in exactly the replicates whose draws include its unit, and the
        # centred products of its plane are bad everywhere (the centre itself is)
        e, row = (0, n // 2) if values == "nan" else (2, n // 3)
        off = boot_np.offsets_of(n, offsets)
        unit = int(np.searchsorted(off, row, side="right") - 1)
        hit = np.concatenate([[True], got["draw_counts"][:, unit] > 0])
        assert 0 < hit[1:].sum() < B                                      # the seed leaves replicates of both kinds
        bad = ~np.isfinite(got["out"][:, 1 + e])
        assert np.array_equal(bad, hit)
        other = [c for c in range(3) if c != e]
        assert np.all(np.isfinite(got["out"][:, [1 + c for c in other]])) and np.all(np.isfinite(got["out"][:, 1 + 3 + 1]) == (e != 1))
        assert not np.any(np.isfinite(got["out"][:, 1 + 3 + (2 if e == 0 else 3)]))
    if values == "equal":                                                 # v - center: the same tiny word in every row; no NaN, no variance
        assert np.all(np.abs(got["unit_mom"][:, 4:]) <= 1e-12)
    if values == "offset":                                                # centred: the products are those of the noise, not 1e12
        assert np.all(np.abs(got["out"][0, 4:]) < 4.0 * n)


def test_two_seeds_differ(cuda):
    planes, pairs, offsets = case(257, "ragged", 3, 1)
    a, b = run(cuda, planes, pairs, offsets, 3, 1), run(cuda, planes, pairs, offsets, 3, 2)
    assert not np.array_equal(a["draw_counts"], b["draw_counts"]) and not np.array_equal(a["out"][1:], b["out"][1:])
    same_bits({k: a[k] for k in ("center", "unit_mom")}, {k: b[k] for k in ("center", "unit_mom")})
    assert np.array_equal(a["out"][0].view(np.uint64), b["out"][0].view(np.uint64))
    c = run(cuda, planes, pairs, offsets, 3, 1 << 32)                     # the high word of the seed is the key's second word
    assert not np.array_equal(a["draw_counts"], c["draw_counts"])


def test_errors_leave_poisoned_outputs_alone(cuda):
    import torch
    from poco_amd import _lib, ops
    n, E, B = 300, 3, 4
    planes = torch.from_numpy(values_of("normal", E, n)).to(cuda)
    pairs = [(0, 1)]
    M = 1 + E + len(pairs)
    mk = lambda: {"center": torch.full((E,), DFILL, device=cuda, dtype=torch.float64),   # noqa: E731
                  "unit_mom": torch.full((n, M), DFILL, device=cuda, dtype=torch.float64),
                  "out": torch.full((B + 1, M), DFILL, device=cuda, dtype=torch.float64),
                  "draw_counts": torch.full((B, n), IFILL, device=cuda, dtype=torch.int32)}
    out = mk()
    small = torch.zeros(ops.bootstrap_scratch_bytes(n, E, 1, n) - 1, device=cuda, dtype=torch.uint8)
    calls = [lambda: ops.bootstrap(planes, pairs, None, B, 0, out=out, scratch=small),
             lambda: ops.bootstrap(planes, [(0, 3)], None, B, 0, out=out),
             lambda: ops.bootstrap(planes, pairs, [0, 100, 90, n], B, 0, out=out),
             lambda: ops.bootstrap(planes, pairs, None, 65537, 0, out=out),
             lambda: ops.bootstrap(planes, pairs, None, B, -1, out=out),
             lambda: ops.bootstrap(planes, pairs, None, B, 0, -1, out=out),
             lambda: ops.bootstrap(planes, pairs, None, B, 0, out=dict(out, center=out["unit_mom"].view(-1)[:E])),
             lambda: ops.bootstrap(planes, pairs, None, B, 0, out=dict(out, out=out["out"][:, :M - 1])),
             lambda: ops.bootstrap(planes[:, ::2], pairs, None, B, 0, out=out)]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.PocoHipError, match="bootstrap"):
            call()
        torch.cuda.synchronize()
        for k, v in out.items():
            assert bool((v == (IFILL if k == "draw_counts" else DFILL)).all()), (i, k)
    res = ops.bootstrap(planes, pairs, None, B, 0, out=out)               # and the same buffers take a good call
    assert res is out and bool((out["draw_counts"].sum(dim=1) == n).all())
