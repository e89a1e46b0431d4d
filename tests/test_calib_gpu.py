"""The calibration operators on the GPU against tests/calib_np.py (include/poco_hip.h poco_op_isotonic / poco_op_calib_apply, DESIGN.md
section 33): the partition, the knot table and the block offsets EXACTLY (tests/test_calib_cpu.py shows that every float input here
decides with a margin; the others are integer-valued), the values within 2^-52 x the block's sum of |y| of math.fsum, every output
bitwise independent of max_blocks and equal from run to run, inputs unchanged, outputs between guard words."""
import functools

import numpy as np
import pytest

from tests import calib_np

T = 2048                                                                  # POCO_ISO_TILE (checked below)
LENGTHS = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 70001)
SEED = 0
U = 2.0 ** -52
G = 64                                                                    # guard words on either side of every output
IFILL, DFILL = -77, -7.25

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name, n):
    """(key, y) of one segment in position order and the yardstick's answer, computed once and left unchanged."""
    key, y = calib_np.pattern(name, n, T, SEED)
    want = calib_np.isotonic(key, y, np.arange(n), [0, n])
    for a in (key, y, *want.values()):
        a.setflags(write=False)
    return key, y, want


def run(cuda, key, y, order, seg, max_blocks=0):
    """One ops.isotonic call into guarded, poisoned outputs -> host arrays.  Checks the guards, the untouched knot rows and that the
    inputs are only read."""
    import torch
    from poco_amd import ops
    N, S = len(order), len(seg) - 1
    dk, dy = torch.from_numpy(np.ascontiguousarray(key)).to(cuda), torch.from_numpy(np.ascontiguousarray(y)).to(cuda)
    do = torch.from_numpy(np.asarray(order, np.int32)).to(cuda)
    ds = torch.from_numpy(np.asarray(seg, np.int32)).to(cuda)
    keep = [t.clone() for t in (dk, dy, do, ds)]
    raw = {"block": torch.full((N + 2 * G,), IFILL, device=cuda, dtype=torch.int32),
           "fit": torch.full((N + 2 * G,), DFILL, device=cuda, dtype=torch.float64),
           "seg_blocks": torch.full((S + 1 + 2 * G,), IFILL, device=cuda, dtype=torch.int32),
           "knots": torch.full((4 * N + 2 * G,), DFILL, device=cuda, dtype=torch.float64)}
    out = {"block": raw["block"][G:G + N], "fit": raw["fit"][G:G + N], "seg_blocks": raw["seg_blocks"][G:G + S + 1],
           "knots": raw["knots"][G:G + 4 * N].view(N, 4)}
    ops.isotonic(dk, dy, do, ds, max_blocks, out=out)
    torch.cuda.synchronize()
    for t, k in zip((dk, dy, do, ds), keep):
        assert torch.equal(t.view(torch.int32), k.view(torch.int32))
    host = {k: v.cpu().numpy() for k, v in raw.items()}
    for k, v in host.items():
        fill = IFILL if v.dtype == np.int32 else DFILL
        assert np.all(v[:G] == fill) and np.all(v[-G:] == fill), k
    res = {"block": host["block"][G:G + N], "fit": host["fit"][G:G + N], "seg_blocks": host["seg_blocks"][G:G + S + 1],
           "knots": host["knots"][G:G + 4 * N].reshape(N, 4)}
    B = int(res["seg_blocks"][S])
    assert 0 <= B <= N and np.all(res["knots"][B:] == DFILL)
    res["knots"] = res["knots"][:B]
    return res


def same_bits(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def check(got, want):
    assert np.array_equal(got["block"], want["block"])
    assert np.array_equal(got["seg_blocks"], want["seg_blocks"])
    assert np.array_equal(got["knots"][:, [0, 1, 3]], want["knots"][:, [0, 1, 3]])
    err = np.abs(got["fit"] - want["fit"])
    print("max |fit - fsum / rows| / (2^-52 sum |y|):", float(np.max(err / (U * np.maximum(want["mag"], 1e-300)), initial=0.0)))
    assert np.all(err <= U * want["mag"])
    heads = np.flatnonzero(got["block"] == np.arange(len(got["block"])))
    assert np.array_equal(got["knots"][:, 2].view(np.uint64), got["fit"][heads].view(np.uint64))      # the table holds the same values
    assert np.array_equal(got["fit"].view(np.uint64), got["fit"][got["block"]].view(np.uint64))       # one value per block


def test_the_tile_is_the_headers():
    from poco_amd import ops
    assert ops.ISO_TILE == T


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", calib_np.PATTERNS)
def test_one_segment(cuda, name, n):
    key, y, want = case(name, n)
    perm = np.random.default_rng(n).permutation(n)                        # rows in any order: position i is row perm[i]
    rk, ry = np.zeros(n, np.float32), np.zeros(n, np.float32)
    rk[perm], ry[perm] = key, y
    if n > 2:
        rk[perm[0]] = -0.0 if key[0] == 0 else rk[perm[0]]                # -0.0 and +0.0 are one key
    got = run(cuda, rk, ry, perm, [0, n])
    check(got, want)
    for mb in (1, 7, 0):
        same_bits(got, run(cuda, rk, ry, perm, [0, n], mb))


@functools.lru_cache(maxsize=None)
def many_segments():
    """Every pattern as a segment of ONE call; empty segments at the start, in the middle and at the end; three segments list the
    same rows (as three maps over one sort do)."""
    keys, ys, orders, seg, base = [], [], [], [0, 0], 0
    for i, name in enumerate(calib_np.PATTERNS):
        n = (T + 1, 3 * T + 17, 65, T - 1)[i % 4]
        key, y = calib_np.pattern(name, n, T, SEED)
        keys.append(key); ys.append(y); orders.append(np.arange(n) + base)
        seg.append(seg[-1] + n)
        if i % 5 == 2:
            seg.append(seg[-1])
        base += n
    for _ in range(2):                                                    # the rows of the last pattern twice more
        orders.append(orders[len(calib_np.PATTERNS) - 1])
        seg.append(seg[-1] + len(orders[-1]))
    seg.append(seg[-1])
    key, y, order = np.concatenate(keys), np.concatenate(ys), np.concatenate(orders)
    return key, y, order, seg, calib_np.isotonic(key, y, order, seg)


def test_all_patterns_as_the_segments_of_one_call(cuda):
    key, y, order, seg, want = many_segments()
    got = run(cuda, key, y, order, seg)
    check(got, want)
    for mb in (1, 7, 0):
        same_bits(got, run(cuda, key, y, order, seg, mb))


def test_4096_tiny_segments(cuda):
    r = np.random.default_rng(4096)
    lens = r.integers(0, 6, 4096)
    seg = np.concatenate([[0], np.cumsum(lens)])
    N = int(seg[-1])
    key = np.concatenate([np.sort(r.integers(0, 3, n)) for n in lens]).astype(np.float32)
    y = r.integers(0, 8, N).astype(np.float32)
    want = calib_np.isotonic(key, y, np.arange(N), seg)
    got = run(cuda, key, y, np.arange(N), seg)
    check(got, want)
    same_bits(got, run(cuda, key, y, np.arange(N), seg, 3))


def test_bad_rows_and_values_stay_inside_the_buffers(cuda):
    """Out-of-range entries of the order and non-finite y: the values are unspecified, but every index the kernels take is clamped
    and every loop is bounded, so the call returns and the guard words (checked by run) are intact."""
    r = np.random.default_rng(9)
    n = T + 300
    key = np.sort(r.gamma(2.0, 0.1, n)).astype(np.float32)
    y = r.gamma(2.0, 0.5, n).astype(np.float32)
    y[r.choice(n, 12, replace=False)] = [np.inf, -np.inf, np.nan] * 4
    order = np.arange(n, dtype=np.int64)
    order[r.choice(n, 9, replace=False)] = [-1, -5, n, n + 100, 2 ** 31 - 1, -2 ** 31, 0, n - 1, 7]
    got = run(cuda, key, y, order, [0, 100, 100, n])
    assert np.all((got["block"] >= 0) & (got["block"] < n)) and len(got["knots"]) >= 2


# ---- poco_op_calib_apply ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def maps():
    """Four maps of 0, 1, 2 and 5000 blocks in one table: lo_b = 3 b, hi_b = 3 b + 1 (b odd: a single key), values increasing."""
    r = np.random.default_rng(5)
    tabs = []
    for B in (0, 1, 2, 5000):
        b = np.arange(B, dtype=np.float64)
        lo = 3.0 * b - 40.0
        tabs.append(np.stack([lo, lo + (b % 2 == 0), np.cumsum(r.uniform(0.01, 1.0, B)) - 3.0, 1 + b % 7], axis=1).reshape(B, 4))
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tabs])]).astype(np.int32)
    return np.concatenate(tabs, axis=0), offs


@pytest.mark.parametrize("S", (1, 27))
@pytest.mark.parametrize("R", (1, 63, 65, 1000))
def test_calib_apply(cuda, R, S):
    import torch
    from poco_amd import ops
    knots, offs = maps()
    r = np.random.default_rng([R, S])
    ids = ((np.arange(S) + 3) % 4).astype(np.int32)                       # S = 1: the map of 5000 blocks
    x = r.uniform(-60.0, 15100.0, (R, S)).astype(np.float32)
    special = r.random((R, S))
    x = np.where(special < 0.25, r.choice(knots[:, :2].reshape(-1), (R, S)).astype(np.float32), x)
    x = np.where((special >= 0.25) & (special < 0.3), r.choice(np.asarray([np.nan, np.inf, -np.inf, -1e30, 1e30, -0.0], np.float32), (R, S)), x)
    x = np.ascontiguousarray(x, np.float32)
    want = calib_np.calib_apply(x, ids, offs, knots)
    raw = torch.full((R * S + 2 * G,), -7.25, device=cuda, dtype=torch.float32)
    dx = torch.from_numpy(x).to(cuda)
    for mb in (0, 1):
        raw.fill_(-7.25)
        ops.calib_apply(dx, torch.from_numpy(ids).to(cuda), torch.from_numpy(offs).to(cuda), torch.from_numpy(knots).to(cuda), mb,
                        out=raw[G:G + R * S].view(R, S))
        torch.cuda.synchronize()
        host = raw.cpu().numpy()
        assert np.all(host[:G] == -7.25) and np.all(host[-G:] == -7.25)
        got = host[G:G + R * S].reshape(R, S)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok].astype(np.float64) - want[ok]) <= np.spacing(np.abs(want[ok])))       # 1 ulp of fp32
        first = np.asarray([knots[offs[m], 0] if offs[m + 1] > offs[m] else np.inf for m in ids])
        last = np.asarray([knots[offs[m + 1] - 1, 1] if offs[m + 1] > offs[m] else -np.inf for m in ids])
        exact = ~ok | (special < 0.3) | (x <= first[None, :]) | (x >= last[None, :])       # at knots, outside the table, NaN: bitwise
        assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32))
    assert np.array_equal(dx.cpu().numpy().view(np.uint32), x.view(np.uint32))
    for c in range(S):                                                    # f is non-decreasing in x
        col = np.argsort(x[:, c], kind="stable")
        v = got[col, c]
        v = v[~np.isnan(v)]
        assert np.all(np.diff(v) >= 0)
