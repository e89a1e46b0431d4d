"""poco_op_rank_curve and poco_op_pearson64 on the GPU against tests/rank_np.py: the order and the midranks element for element,
the cut sums within the fp64 bound of their length, the cut keys bit for bit, everything bitwise independent of the grid and
repeatable, inputs only read, argument errors before any GPU work (include/poco_hip.h)."""
import functools

import numpy as np
import pytest
import scipy.stats
import torch

from poco_amd import _lib, ops
from tests import rank_np

pytestmark = pytest.mark.gpu
T = ops.RANK_TILE
U = 2.0 ** -52
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 70001]
EIGHT = np.asarray([-3.5, -1.0, -1e-45, 0.0, 1e-45, 0.25, 2.0, 1e30], np.float32)


def _bits(n, f):
    return np.asarray([f(i) for i in range(n)], np.uint32).view(np.float32)


def _mix(i):
    return (i * 2654435761) & 0xffffffff


KEYSETS = {
    "normal": lambda n, r: r.standard_normal(n).astype(np.float32),
    "equal": lambda n, r: np.full(n, 0.37, np.float32),
    "low_byte": lambda n, r: _bits(n, lambda i: 0x3f800000 | (_mix(i) >> 24)),                # three passes see one digit
    "high_byte": lambda n, r: _bits(n, lambda i: ((_mix(i) >> 25) << 24) | 0x00123456),       # positive, finite: top byte 0..127
    "negative": lambda n, r: (-np.abs(r.standard_normal(n)) - 0.5).astype(np.float32),
    "mixed_sign": lambda n, r: np.round(r.standard_normal(n) * 4).astype(np.float32),
    "zeros": lambda n, r: np.where(np.arange(n) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32),
    "inf": lambda n, r: r.choice(np.asarray([-np.inf, np.inf, -1.0, 0.5], np.float32), n),
    "denormal": lambda n, r: _bits(n, lambda i: ((_mix(i) >> 31) << 31) | (_mix(i + 7) >> 12 & 0x7ff)),
    "nan": lambda n, r: _bits(n, lambda i: (0x7fc00000, 0xffc00001, 0x7f800123, 0x3f800000, 0xbf800000)[_mix(i) % 5]),
    "sorted": lambda n, r: np.sort(r.standard_normal(n).astype(np.float32)),
    "reversed": lambda n, r: np.sort(r.standard_normal(n).astype(np.float32))[::-1].copy(),
    "eight": lambda n, r: EIGHT[np.arange(n) % 8],                                           # groups straddle every border and cut
    "missing_digit": lambda n, r: _bits(n, lambda i: 0x40000000 | ((_mix(i) >> 20 & 0x7f) * 2 << 8) | (_mix(i) >> 28 << 1)),
}
# K and E walk through every pair while the cases go by; K = 1024 needs a yardstick of 1025 exact sums, so it stays with the small n
# (and test_k_1024_at_a_size_of_several_tiles), and the largest n stops at one value plane for the same reason
PAIRS = [(K, E) for K in (1, 7, 20, 1024) for E in (0, 1, 4)]
CASES = [(name, n) for name in KEYSETS for n in SIZES]


def pick(i, n):
    K, E = PAIRS[i % len(PAIRS)]
    return (K if K < 1024 or n <= T + 1 else 20), (E if n <= 3 * T + 17 else min(E, 1))


@functools.lru_cache(maxsize=None)
def case(name, n):
    """Keys, five value planes and the yardstick's order and midranks of one case: computed once, shared, never written to."""
    r = np.random.default_rng(SIZES.index(n) * 100 + list(KEYSETS).index(name))
    key = np.ascontiguousarray(KEYSETS[name](n, r), np.float32)
    assert key.shape == (n,)
    vals = np.ascontiguousarray(np.stack([np.abs(r.standard_normal(n)), r.standard_normal(n) * 1e3, r.uniform(0, 1e-3, n),
                                          np.round(r.standard_normal(n)), np.full(n, 0.1)]).astype(np.float32))
    for a in (key, vals):
        a.setflags(write=False)
    order = rank_np.stable_order(key)
    return key, vals, order, rank_np.midranks(key, order)


def dev(a, cuda):
    """A device copy of a (read-only) host array."""
    return torch.tensor(a, device=cuda)


def run(cuda, key, vals, K, max_blocks=0):
    out = ops.rank_curve(dev(key, cuda), None if vals is None else dev(vals, cuda), K, max_blocks)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("order", "rank", "cuts", "cut_keys"))


@pytest.mark.parametrize("i,name,n", [(i, name, n) for i, (name, n) in enumerate(CASES)], ids=[f"{name}-{n}" for name, n in CASES])
def test_order_ranks_cuts_and_cut_keys(cuda, i, name, n):
    key, vals5, order, rank = case(name, n)
    K, E = pick(i, n)
    vals = vals5[:E] if E else None
    dk = dev(key, cuda)
    dv = dev(vals, cuda) if E else None
    got = {k: v.cpu().numpy() for k, v in ops.rank_curve(dk, dv, K).items()}
    assert np.array_equal(dk.cpu().numpy().view(np.uint32), key.view(np.uint32))               # the inputs are only read
    assert dv is None or np.array_equal(dv.cpu().numpy().view(np.uint32), vals.view(np.uint32))
    assert got["order"].dtype == np.int32 and np.array_equal(got["order"], order)
    assert np.array_equal(got["order"], np.argsort(key, kind="stable"))
    assert got["rank"].dtype == np.float64 and np.array_equal(got["rank"], rank)
    if name == "equal":
        assert np.array_equal(got["order"], np.arange(n)) and np.all(got["rank"] == (n + 1) / 2)
    if name != "nan":
        cuts, mags, cut_keys = rank_np.cut_sums(key, vals, K, order)
        assert got["cuts"].shape == (E + 1, K + 1) and got["cut_keys"].shape == (K + 1,)
        fin = np.isfinite(cuts)
        assert np.all(np.isfinite(got["cuts"][fin]))
        off = np.abs(got["cuts"][fin] - cuts[fin])
        print(f"{name} n={n} K={K} E={E}: worst |cut - fsum| / (n 2^-52 sum|v|) =",
              float(np.max(off / np.maximum(n * U * mags[fin], 1e-300), initial=0.0)))
        assert np.all(off <= n * U * mags[fin])                                             # the fp64 bound of a sum of n terms
        assert np.array_equal(got["cuts"][~fin], cuts[~fin], equal_nan=True)
        assert np.array_equal(got["cut_keys"].view(np.uint32), cut_keys.view(np.uint32))
    for mb in (1, 7, 0):                                                                    # any grid, any run: the same bits
        assert same_bits(got, run(cuda, key, vals, K, mb)), mb


def test_k_1024_at_a_size_of_several_tiles(cuda):
    """Every cut of K = 1024 inside 3 T + 17 rows: cut positions in every tile, most of them off the tile borders."""
    n = 3 * T + 17
    key, vals5, _, _ = case("eight", n)
    vals = vals5[:1]
    got = run(cuda, key, vals, 1024)
    cuts, mags, cut_keys = rank_np.cut_sums(key, vals, 1024)
    assert np.all(np.abs(got["cuts"] - cuts) <= n * U * mags)
    assert np.array_equal(got["cut_keys"].view(np.uint32), cut_keys.view(np.uint32))
    for mb in (1, 7):
        assert same_bits(got, run(cuda, key, vals, 1024, mb))


def test_outputs_into_guarded_buffers_and_a_larger_scratch(cuda):
    """Nothing is written outside the four outputs, and a scratch buffer larger than asked for, full of NaN, changes nothing."""
    n, K, E = T + 65, 7, 1
    key, vals5, order, rank = case("mixed_sign", T + 1)
    key, vals = np.concatenate([key, key[:64]]), np.concatenate([vals5[:1], vals5[:1, :64]], axis=1)
    want = run(cuda, key, vals, K)
    G = 64
    wide = {"order": torch.full((n + 2 * G,), -77, dtype=torch.int32, device=cuda), "rank": torch.full((n + 2 * G,), -77.0, dtype=torch.float64, device=cuda),
            "cuts": torch.full(((E + 1) * (K + 1) + 2 * G,), -77.0, dtype=torch.float64, device=cuda),
            "cut_keys": torch.full((K + 1 + 2 * G,), -77.0, dtype=torch.float32, device=cuda)}
    out = {k: v[G:-G].view(want[k].shape) for k, v in wide.items()}
    scratch = torch.full((ops.rank_curve_scratch_bytes(n, E) + 4096,), 0xff, dtype=torch.uint8, device=cuda)
    ops.rank_curve(dev(key, cuda), dev(vals, cuda), K, out=out, scratch=scratch)
    assert same_bits(want, {k: v.cpu().numpy() for k, v in out.items()})
    for k, v in wide.items():
        assert bool((v[:G] == -77).all()) and bool((v[-G:] == -77).all()), k
    assert bool((scratch[-4096:] == 0xff).all())


def test_argument_errors_leave_the_outputs_untouched(cuda):
    n, K, E = 300, 7, 2
    key = torch.arange(n, dtype=torch.float32, device=cuda)
    vals = torch.ones(E, n, dtype=torch.float32, device=cuda)
    out = {"order": torch.full((n,), -77, dtype=torch.int32, device=cuda), "rank": torch.full((n,), -77.0, dtype=torch.float64, device=cuda),
           "cuts": torch.full((E + 1, K + 1), -77.0, dtype=torch.float64, device=cuda), "cut_keys": torch.full((K + 1,), -77.0, dtype=torch.float32, device=cuda)}
    scratch = torch.zeros(ops.rank_curve_scratch_bytes(n, E), dtype=torch.uint8, device=cuda)
    fn = _lib.lib().poco_op_rank_curve
    fn.argtypes = ops.RANK_ARGTYPES
    p = lambda t: t.data_ptr()   # noqa: E731
    good = dict(key=p(key), vals=p(vals), n=n, E=E, K=K, scratch=p(scratch), room=scratch.numel(), order=p(out["order"]), rank=p(out["rank"]),
                cuts=p(out["cuts"]), cut_keys=p(out["cut_keys"]), mb=0)
    bad = [dict(key=None), dict(vals=None), dict(scratch=None), dict(order=None), dict(rank=None), dict(cuts=None), dict(cut_keys=None),
           dict(n=0), dict(n=(1 << 24) + 1), dict(E=-1), dict(E=5), dict(K=0), dict(K=1025), dict(room=good["room"] - 1), dict(room=0), dict(mb=-1),
           dict(order=good["key"]), dict(rank=good["vals"]), dict(cut_keys=good["key"] + 4 * (n - 1)), dict(cuts=good["rank"]),
           dict(rank=good["order"] + 8), dict(scratch=good["vals"]), dict(order=good["scratch"] + 256)]
    for kw in bad:
        a = dict(good, **kw)
        rc = fn(a["key"], a["vals"], a["n"], a["E"], a["K"], a["scratch"], a["room"], a["order"], a["rank"], a["cuts"], a["cut_keys"], a["mb"],
                _lib.current_stream())
        assert rc == 1, kw
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v == -77).all()), k
    with pytest.raises(_lib.PocoHipError, match="K must be in"):
        ops.rank_curve(key, vals, 0)
    with pytest.raises(_lib.PocoHipError, match="vals"):
        ops.rank_curve(key, vals[:, :-1].contiguous(), 7)
    with pytest.raises(_lib.PocoHipError, match="scratch"):
        ops.rank_curve(key, vals, 7, scratch=scratch[:-1])


# ---- poco_op_pearson64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 65, T + 1, 70001])
def test_pearson64_on_ranks_is_spearman(cuda, n):
    a, vals5, _, rank_a = case("mixed_sign", n)                             # heavy ties
    b = (a + vals5[3]).astype(np.float32)
    ra = ops.rank_curve(dev(a, cuda), None, 1)["rank"]
    rb = ops.rank_curve(dev(b, cuda), None, 1)["rank"]
    assert np.array_equal(ra.cpu().numpy(), rank_a)
    rho = [float(ops.pearson64(ra, rb, mb).cpu()[0]) for mb in (0, 1, 7, 0)]
    if np.all(a == a[0]) or np.all(b == b[0]):
        assert all(np.isnan(x) for x in rho)
        return
    want = scipy.stats.spearmanr(a, b)[0]
    print(f"n={n}: |rho - scipy| / 2^-52 = {abs(rho[0] - want) / U}")
    assert abs(rho[0] - want) <= 64 * U
    assert len({np.float64(x).tobytes() for x in rho}) == 1                  # any grid, any run: the same bits
    assert abs(rho[0] - rank_np.pearson(ra.cpu().numpy(), rb.cpu().numpy())) <= 64 * U


def test_pearson64_constant_clip_and_untouched_inputs(cuda):
    x = torch.linspace(-3, 5, 1000, dtype=torch.float64, device=cuda)
    keep = x.clone()
    for const in (torch.full_like(x, 0.1), torch.zeros_like(x), torch.full_like(x, 1e300)):
        assert np.isnan(float(ops.pearson64(x, const).cpu()[0])) and np.isnan(float(ops.pearson64(const, x).cpu()[0]))
    up, down = float(ops.pearson64(x, x).cpu()[0]), float(ops.pearson64(x, -x).cpu()[0])
    assert 1.0 - 4 * U <= up <= 1.0 and -1.0 <= down <= -1.0 + 4 * U and down == -up                        # clipped, never beyond
    assert abs(float(ops.pearson64(x, 3.0 * x + 2.0).cpu()[0]) - 1.0) <= 64 * U
    assert torch.equal(x, keep)
    one = torch.ones(1, dtype=torch.float64, device=cuda)
    assert np.isnan(float(ops.pearson64(one, one).cpu()[0]))                 # n = 1: constant
    guard = torch.full((3,), -77.0, dtype=torch.float64, device=cuda)
    ops.pearson64(x, -x, out=guard[1:2])
    assert guard.cpu().tolist() == [-77.0, down, -77.0]
    fn = _lib.lib().poco_op_pearson64
    fn.argtypes = ops.PEARSON64_ARGTYPES
    for args in ((None, x.data_ptr(), 10, guard.data_ptr(), 0), (x.data_ptr(), x.data_ptr(), 0, guard.data_ptr(), 0),
                 (x.data_ptr(), x.data_ptr(), 10, x.data_ptr() + 8, 0), (x.data_ptr(), x.data_ptr(), 10, guard.data_ptr(), -1)):
        assert fn(*args, _lib.current_stream()) == 1
    torch.cuda.synchronize()
    assert guard.cpu().tolist() == [-77.0, down, -77.0] and torch.equal(x, keep)
    with pytest.raises(_lib.PocoHipError, match="one length"):
        ops.pearson64(x, x[:-1].contiguous())
