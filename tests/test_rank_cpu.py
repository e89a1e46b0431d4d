"""Rank-based uncertainty metrics without a GPU: the yardstick tests/rank_np.py against numpy and scipy, poco_amd/ranking.py against
the yardstick on identical cut sums, two hand-made rankings with known answers, the C ABI's declarations and argument checks, and
eval.py's flags (include/poco_hip.h poco_op_rank_curve)."""
import importlib.util
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import pytest
import scipy.stats

from poco_amd import _lib, ranking
from tests import rank_np

ROOT = Path(__file__).resolve().parent.parent
U = 2.0 ** -52


def tied_keys(seed, n):
    """Seeded float32 keys with ties, both zeros, infinities, a denormal and NaNs of both signs."""
    r = np.random.default_rng(seed)
    k = np.round(r.standard_normal(n), 1).astype(np.float32)
    k[r.choice(n, n // 10, replace=False)] = 0.0
    k[r.choice(n, n // 10, replace=False)] = -0.0
    for v in (np.inf, -np.inf, 1e-45, -1e-45):
        k[r.integers(n)] = v
    k[r.choice(n, 3, replace=False)] = np.nan
    bits = k.view(np.uint32)
    bits[np.flatnonzero(np.isnan(k))[0]] = 0xffc00001                     # a negative NaN with a payload
    return k


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n", [(0, 1), (1, 2), (2, 97), (3, 1000)])
def test_yardstick_order_and_midranks_are_numpy_and_scipy(seed, n):
    k = tied_keys(seed, max(n, 40))[:n]
    assert np.array_equal(rank_np.stable_order(k), np.argsort(k, kind="stable"))
    finite = k[~np.isnan(k)]
    if len(finite):
        assert np.array_equal(rank_np.midranks(finite), scipy.stats.rankdata(finite, method="average"))
    nan = np.isnan(k)
    if nan.any():                                                        # every NaN is one key: they tie, behind everything else
        assert np.all(rank_np.midranks(k)[nan] == len(finite) + 0.5 * (nan.sum() + 1))


def test_yardstick_canonical_keys():
    k = np.asarray([-0.0, 0.0, np.nan, 1.0], np.float32)
    k.view(np.uint32)[2] = 0xff800001
    assert rank_np.bits32(rank_np.canonical(k)).tolist() == [0, 0, 0x7fc00000, 0x3f800000]
    img = rank_np.sort_image(np.asarray([-np.inf, -1.0, -1e-45, 0.0, 1e-45, 1.0, np.inf, np.nan], np.float32))
    assert np.all(np.diff(img.astype(np.int64)) > 0)


def test_yardstick_spearman_is_scipy():
    r = np.random.default_rng(5)
    a = np.round(r.standard_normal(500), 1).astype(np.float32)
    b = (a + np.round(r.standard_normal(500), 1)).astype(np.float32)
    want = scipy.stats.spearmanr(a, b)[0]
    assert abs(rank_np.spearman(a, b) - want) <= 64 * U
    assert np.isnan(rank_np.spearman(a, np.ones(500, np.float32)))


def test_yardstick_cut_sums():
    key = np.asarray([3, 1, 2, 1, 5, 4], np.float32)
    err = np.asarray([30, 10, 20, 11, 50, 40], np.float32)
    cuts, mags, cut_keys = rank_np.cut_sums(key, [err], 3)
    assert cuts.tolist() == [[0, 2, 7, 16], [0, 21, 71, 161]] and np.array_equal(cuts, mags)
    assert cut_keys.tolist() == [1, 1, 3, 5]
    cuts, _, cut_keys = rank_np.cut_sums(key[:2], None, 5)                 # K > n: c = 0 0 0 1 1 2
    assert cuts.tolist() == [[0, 0, 0, 1, 1, 4]] and cut_keys.tolist() == [1, 1, 1, 1, 1, 3]


# ---- poco_amd/ranking.py against the yardstick on identical cuts -----------------------------------------------------------------------
def close(got, want, mags, K):
    """|got - want| <= (K + 2) 2^-52 x the sum of the absolute terms that enter: the fp64 bound for sums of that length."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= (K + 2) * U * np.broadcast_to(mags, want.shape)[ok]), np.abs(got - want)[ok].max()


@pytest.mark.parametrize("n,K", [(1000, 20), (1000, 7), (1000, 1), (5, 7), (300, 1024)])
def test_host_functions_match_the_yardstick(n, K):
    r = np.random.default_rng(n + K)
    key = np.abs(np.round(r.standard_normal(n), 2)).astype(np.float32)
    errs = [np.abs(key * 0.1 + 0.05 * r.standard_normal(n)).astype(np.float32), r.uniform(0.01, 1, n).astype(np.float32)]
    cuts, mags, cut_keys = rank_np.cut_sums(key, errs, K)
    assert ranking.cut_counts(n, K).tolist() == rank_np.cut_counts(n, K)
    cnt = np.maximum(np.asarray(rank_np.cut_counts(n, K), np.float64), 1.0)
    for e in (1, 2):
        curve = ranking.sparsification(cuts[e], n)
        want = rank_np.sparsification(cuts[e], n)
        close(curve, want, (mags[e] / cnt)[:0:-1], K)
        oracle_cuts = rank_np.cut_sums(errs[e - 1], None, K)[0][0]
        oracle = ranking.sparsification(oracle_cuts, n)
        close(oracle, rank_np.sparsification(oracle_cuts, n), (mags[e] / cnt)[:0:-1], K)
        # areas: K terms, each at most (|curve| + |oracle|) / mean / K
        scale = (np.nansum(np.abs(want)) + np.nansum(np.abs(oracle))) / abs(want[0]) / K
        close(ranking.ause(curve, oracle), rank_np.ause(want, rank_np.sparsification(oracle_cuts, n)), scale, K)
        close(ranking.aurg(curve), rank_np.aurg(want), scale + 1.0, K)
    bins = np.maximum(np.diff(rank_np.cut_counts(n, K)), 1)[:, None]
    close(ranking.reliability(cuts, n), rank_np.reliability(cuts, n),
          np.concatenate([np.ones((K, 1)), ((mags[:, 1:] + mags[:, :-1]) / bins.T).T], axis=1), K)
    close(ranking.threshold_table(cut_keys, cuts, n), rank_np.threshold_table(cut_keys, cuts, n),
          np.concatenate([np.ones((K, 2)), (mags[1:, 1:] / cnt[1:]).T], axis=1), K)


def curves(key, err, K):
    n = len(key)
    curve = ranking.sparsification(rank_np.cut_sums(key, [err], K)[0][1], n)
    oracle = ranking.sparsification(rank_np.cut_sums(err, None, K)[0][0], n)
    return curve, oracle


def test_a_perfect_ranking_has_ause_zero_and_a_reversed_one_negative_aurg():
    err = np.arange(1, 41, dtype=np.float32)
    curve, oracle = curves(err.copy(), err, 10)                           # the uncertainty orders the rows as the error does
    assert np.array_equal(curve, oracle) and ranking.ause(curve, oracle) == 0.0 and ranking.aurg(curve) > 0
    # by hand: keeping the c smallest of 1..40 has mean (c + 1) / 2; all rows: 20.5; trapezoid over k / 10, k = 0..9
    want = [(40 - 4 * k + 1) / 2 for k in range(10)]
    assert curve.tolist() == want
    assert abs(ranking.aurg(curve) - sum(0.5 * ((20.5 - a) + (20.5 - b)) for a, b in zip(want, want[1:])) / 20.5 / 10) <= 12 * U
    curve, oracle = curves(-err, err, 10)                                 # the most certain rows are the worst ones
    assert ranking.aurg(curve) < 0 and ranking.ause(curve, oracle) > 0
    assert abs(ranking.aurg(curve) + ranking.aurg(oracle)) <= 12 * U * 2     # mirrored around the constant curve
    assert abs(ranking.ause(curve, oracle) - (ranking.aurg(oracle) - ranking.aurg(curve))) <= 12 * U * 2
    assert abs(rank_np.spearman(-err, err) + 1.0) <= 4 * U and abs(rank_np.spearman(err, err) - 1.0) <= 4 * U


def test_a_single_cut_has_no_area():
    err = np.arange(1, 9, dtype=np.float32)
    curve, oracle = curves(err, err, 1)
    assert curve.tolist() == [4.5] and ranking.ause(curve, oracle) == 0.0 and ranking.aurg(curve) == 0.0


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("poco_op_rank_curve", "poco_op_rank_curve_scratch_bytes", "poco_op_pearson64", "poco_evaluator_rank_inputs")


def test_header_declares_and_library_exports_the_new_symbols():
    from poco_amd import ops
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.header_symbols() and hasattr(L, s), s
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and L.poco_abi_version() == 4                       # additions only
    assert f"#define POCO_RANK_TILE {ops.RANK_TILE}\n" in txt
    assert ops.RANK_TILE % 256 == 0


def test_scratch_query():
    from poco_amd import ops
    q = ops.rank_curve_scratch_bytes
    assert q(0, 0) == 0 and q(-1, 1) == 0 and q((1 << 24) + 1, 0) == 0 and q(10, -1) == 0 and q(10, 5) == 0
    assert 0 < q(1, 0) <= q(1, 4) and q(1000, 1) < q(100000, 1) < q(1 << 24, 4) < 1 << 30
    assert q(ops.RANK_TILE, 1) < q(ops.RANK_TILE + 1, 1)                  # one more tile
    assert q(12345, 2) == q(12345, 2) and q(12345, 2) % 256 == 0


def test_rank_curve_refuses_bad_arguments_before_any_gpu_work():
    from poco_amd import ops
    L = _lib.lib()
    fn = L.poco_op_rank_curve
    fn.argtypes = ops.RANK_ARGTYPES
    MB = 1 << 26                                                         # fake device pointers, far enough apart not to overlap
    key, vals, scratch, order, rank, cuts, cut_keys = (MB * i for i in range(1, 8))
    n = 5000
    room = ops.rank_curve_scratch_bytes(n, 4)

    def call(key=key, vals=vals, n=n, E=2, K=20, scratch=scratch, room=room, order=order, rank=rank, cuts=cuts, cut_keys=cut_keys, mb=0):
        return fn(key, vals, n, E, K, scratch, room, order, rank, cuts, cut_keys, mb, None)
    bad = [dict(key=None), dict(vals=None), dict(scratch=None), dict(order=None), dict(rank=None), dict(cuts=None), dict(cut_keys=None),
           dict(n=0), dict(n=-3), dict(n=(1 << 24) + 1), dict(E=-1), dict(E=5), dict(K=0), dict(K=-1), dict(K=1025), dict(mb=-1),
           dict(room=0), dict(room=ops.rank_curve_scratch_bytes(n, 2) - 1), dict(rank=rank + 4), dict(cuts=cuts + 4), dict(scratch=scratch + 4),
           dict(order=key), dict(order=key + 4 * (n - 1)), dict(rank=vals + 4 * n), dict(cuts=key), dict(cut_keys=vals + 8 * n - 4),
           dict(scratch=key - 256), dict(scratch=vals), dict(rank=order), dict(cuts=rank + 8 * (n - 1)), dict(cut_keys=cuts + 8 * 3 * 21 - 4),
           dict(order=scratch + 1024), dict(cut_keys=scratch + 512)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "poco_op_rank_curve" in L.poco_last_error().decode(), kw
    p = L.poco_op_pearson64
    p.argtypes = ops.PEARSON64_ARGTYPES
    x, y, r = MB, 2 * MB, 3 * MB
    for args in ((None, y, 10, r, 0), (x, None, 10, r, 0), (x, y, 10, None, 0), (x, y, 0, r, 0), (x, y, (1 << 24) + 1, r, 0), (x, y, 10, r, -1),
                 (x + 4, y, 10, r, 0), (x, y, 10, r + 4, 0), (x, y, 10, x + 8, 0), (x, y, 10, y + 72, 0)):
        assert p(*args, None) == 1, args
        assert "poco_op_pearson64" in L.poco_last_error().decode(), args


def test_evaluator_rank_inputs_refuses_bad_arguments_before_any_gpu_work():
    import ctypes as C
    from poco_amd import evaluate
    L = evaluate._bind()
    fn = L.poco_evaluator_rank_inputs
    hn, hE = C.c_int64(-7), C.c_int(-7)
    assert fn(None, 0, 1 << 26, 1 << 27, 10, C.byref(hn), C.byref(hE), None) == 1
    Jr = np.eye(3, 50, dtype=np.float32)
    h = C.c_void_p()
    assert L.poco_evaluator_create(Jr.ctypes.data, 3, 50, np.arange(3, dtype=np.int32).ctypes.data, 3, 0, None, 0, 1, 8, C.byref(h)) == 0
    try:
        for mode, key, vals, n, e in ((2, 1 << 26, 1 << 27, hn, hE), (-1, 1 << 26, 1 << 27, hn, hE), (0, None, 1 << 27, hn, hE),
                                      (0, 1 << 26, None, hn, hE), (1, 1 << 26, 1 << 27, None, hE), (1, 1 << 26, 1 << 27, hn, None)):
            assert fn(h, mode, key, vals, 10, C.byref(n) if n is not None else None, C.byref(e) if e is not None else None, None) == 1
            assert "poco_evaluator_rank_inputs" in L.poco_last_error().decode()
        assert fn(h, 0, 1 << 26, 1 << 27, 10, C.byref(hn), C.byref(hE), None) == 3          # POCO_ERR_STATE: no record yet
        assert (hn.value, hE.value) == (-7, -7)
    finally:
        L.poco_evaluator_destroy(h)


def test_ops_refuse_host_tensors_and_bad_shapes_without_a_gpu():
    import torch
    from poco_amd import ops
    with pytest.raises(_lib.PocoHipError, match="rank_curve.*CUDA"):
        ops.rank_curve(torch.zeros(8))
    with pytest.raises(_lib.PocoHipError, match="pearson64.*CUDA"):
        ops.pearson64(torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64))


# ---- eval.py --------------------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]


def _one_sentence(msg, word):
    assert word in msg and msg.count(". ") == 0 and "\n" not in msg, msg


def test_eval_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    spec = importlib.util.spec_from_file_location("poco_eval_cli_rank", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = BASE + ["--j_regressor", "none.npy", "--dataset", str(tmp_path / "missing.npz")]
    a = cli.parse_args(base)
    assert a.rank_metrics is False and a.rank_bins is None
    a = cli.parse_args(base + ["--rank_metrics", "--rank_bins", "50"])
    assert a.rank_metrics is True and a.rank_bins == 50
    R = ["--rank_metrics"]
    for flags, word in ((["--rank_bins", "20"], "needs --rank_metrics"), (R + ["--rank_bins", "0"], "1..1024"), (R + ["--rank_bins", "1025"], "1..1024"),
                        (R + ["--rank_bins", "-4"], "1..1024"), (R + ["--segm"], "--segm"), (R + ["--likelihood"], "--likelihood"),
                        (R + ["--cfg2", "configs/demo_poco_pare.yaml", "--ckpt2", "x.pt"], "--cfg2"),
                        (R + ["--tta", "flip", "--crop", "dataset"], "--tta")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work, before the dataset file is looked at
            cli.main(cli.parse_args(base + flags))
        _one_sentence(str(e.value), word)
        assert "--rank_metrics" in str(e.value) or "--rank_bins" in str(e.value), (flags, e.value)
        assert "missing.npz" not in str(e.value), (flags, e.value)
    for ok in (R, R + ["--rank_bins", "1"], R + ["--rank_bins", "1024"]):
        with pytest.raises(SystemExit, match="missing.npz"):                     # flags that may run get as far as the dataset file
            cli.main(cli.parse_args(base + ok))


def test_flag_error_sentences():
    assert ranking.flag_error(NS()) is None and ranking.flag_error(NS(rank_metrics=True, rank_bins=None)) is None
    assert ranking.flag_error(NS(rank_metrics=True, rank_bins=1024)) is None
    _one_sentence(ranking.flag_error(NS(rank_metrics=False, rank_bins=3)), "--rank_bins")
    _one_sentence(ranking.flag_error(NS(rank_metrics=True, likelihood=True)), "--likelihood")


def test_npz_key_names():
    assert len(ranking.RANK_NPZ_KEYS) == 12 and len(set(ranking.RANK_NPZ_KEYS)) == 12
    assert all(k.startswith(("rank_spars_", "rank_oracle_", "rank_reliab_")) or k in ("rank_thresholds", "rank_summary") for k in ranking.RANK_NPZ_KEYS)
    assert ranking.RANK_SUMMARY_FIELDS[0] == "K" and len(ranking.RANK_SUMMARY_FIELDS) == 13
